"""Planted graphs for the map kernels of the rectangle and the house (csrc/gm_mine.hip: rect_lds_kernel + rect_acc_kernel, house_lds_kernel +
house_acc_kernel): every cell puts a packed counter on the last value its width holds, or a centre, a row or an end on one side of a size at
which the kernels change path (test helper; imported by tests/test_map_probe_graphs_host.py and tests/test_gpu_map_kernels.py).  Graphs are
made with numpy alone; the one thing taken from the package is the Graph CONTAINER.  Expected counts: tests/rect_local_ref.py and
tests/house_ref.py, which know nothing of centres, ranges or widths.

Every size comes from the library (gm_constant "map_*", handed in as `c`: graphminer_amd.map_constants()), none is written here:
  rect_block      ids of a block of 32-bit counters; a range of 8- / 16-bit counters covers 4 / 2 blocks
  one_task_rows   rows up to which a centre is ONE task (v, -1) that keeps a row per thread; above: a task (v, k) per range
  long_row        keys of a row inside a range from which a wave strides the row instead of flattening it
  tile_group, mark_window   keys a wave requests together / flattened positions per owner-mark window
  house_ids       ids per range of the house
  house_fw16_rows rows up to which a one-task centre of the house packs two ends into a word (four ranges per walk; above: two)
  house_wg_row, house_wg_queue   keys from which a row of a one-task centre is shared out to the workgroup; slots of that queue
  heavy_centre    2-paths from which a centre of the acc kernels gets a whole workgroup
  lds_min_default, house_walk_min_default   2-paths from which a centre counts in the LDS maps, and per walk of a one-task centre of the house,
                  where no developer option says otherwise

rect_plan / house_plan restate, from the CSR and those sizes alone, the plan the library builds (csrc/gm_centre_plan.h) in the form of
graphminer_amd.map_plan_info: the GPU test holds the two against each other BEFORE it compares a count, so a cell that lands on another path
fails.  The rectangle runs by default on the copy numbered ascending in (degree, id) -- planted_squares.degree_copy says where that puts a
vertex -- and under GM_T6_AS_NUMBERED on the graph as given; the house runs as given.  A cell is (graph, options, claims): `claims` maps a
sentence about the path to a bool worked out here on the CPU; every one must hold."""
from __future__ import annotations

from dataclasses import dataclass, field
from math import comb

import numpy as np

from planted_squares import _graph, degree_copy

HUB_ROWS = 2 ** 8 + 44    # rows of a hub whose degree must need 16-bit counters (any number from 2^8 on)
CUT_MARGIN = 1000         # ids of the degree-2 zone between its first gadget and the ends below the cut (any number that leaves room)
ROW_WEIGHT = 8            # d(x) + 1 of the rows under the two centres placed on heavy_centre: heavy_centre / ROW_WEIGHT rows each
LANES = 64   # lanes of a wave: a one-task centre deals row r to wave r mod (one_task_rows / LANES)



# ---- the plans, restated ------------------------------------------------------------------------------------------------------------------
def _csr(g):
    rp = np.asarray(g.row_ptr, dtype=np.int64)
    col = np.asarray(g.col_idx, dtype=np.int64)
    src = np.repeat(np.arange(rp.size - 1, dtype=np.int64), np.diff(rp))
    return rp, col, src


def rect_ranges(nv, deg, c, max_ranges=None):
    """(rb[0 .. n], lb[0 .. n)) of rect_lds_ranges: from the last id down, 8 / 16 bits while the next 4 / 2 blocks hold no degree of 2^8 / 2^16"""
    W = c["rect_block"]
    nblk = (nv + W - 1) // W
    bmax = np.zeros(max(nblk, 1), dtype=np.int64)
    if nv:
        np.maximum.at(bmax, (nv - 1 - np.arange(nv)) // W, deg)
    rb, lb, blk, hi = [nv], [], 0, nv
    while hi > 0 and (max_ranges is None or len(lb) < max_ranges):
        w = 3 if bmax[blk:blk + 4].max(initial=0) < 2 ** 8 else 4 if bmax[blk:blk + 2].max(initial=0) < 2 ** 16 else 5
        blk += 1 << (5 - w)
        hi = max(0, hi - (W << (5 - w)))
        lb.append(w)
        rb.append(hi)
    return rb[::-1], lb[::-1]


def _task_counts(lds, rows, ntasks_per_range_centre, front_key, front_all, rest_work, c):
    T, heavy = c["one_task_rows"], c["heavy_centre"]
    per_range = lds & (rows > T)
    front = front_key[lds & (front_all | (front_key > 0))]
    fh, rh = int((front >= heavy).sum()), int((rest_work >= heavy).sum())
    fl, rl = (front.size - fh + 3) // 4, (rest_work.size - rh + 3) // 4
    return {"lds_range_tasks": int(ntasks_per_range_centre[per_range].sum()), "lds_whole_tasks": int((lds & (rows <= T)).sum()),
            "front_tasks": fh + fl, "front_heavy_tasks": fh, "heavy_tasks": fh + rh, "light_tasks": fl + rl}


def rect_plan(g, c, lds_min=None, max_ranges=None):
    """the plan of ensure_rect_plan on g AS NUMBERED, in map_plan_info's form (plus "idx0" and "lds": the centres that count in LDS)"""
    rp, col, src = _csr(g)
    nv, deg = rp.size - 1, np.diff(rp)
    rb, lb = rect_ranges(nv, deg, c, max_ranges)
    cut = rb[0]
    lds_min = c["lds_min_default"] if lds_min is None else lds_min   # (no GM_RECT_LDS_MIN given)
    below = col < src
    idx0 = np.bincount(src[below], minlength=nv)
    # a centre's 2-path estimate: its neighbours x below it, d(x) + 1 each; of those the keys of row x below the cut
    keys_below_cut = np.bincount(src[col < cut], minlength=nv)
    work = np.bincount(src[below], weights=(deg[col[below]] + 1), minlength=nv).astype(np.int64)
    wcut = np.bincount(src[below], weights=keys_below_cut[col[below]], minlength=nv).astype(np.int64)
    lds = (work > 0) & (work >= lds_min) & (np.arange(nv) > cut)
    top = np.searchsorted(np.asarray(rb[1:max(len(lb), 1)]), np.arange(nv) - 1, side="right")  # the range that holds v - 1
    out = {"n": len(lb), "cut": cut, "rb": rb, "lb": lb, "idx0": idx0, "lds": lds, "work": work, "wcut": wcut}
    out.update(_task_counts(lds, idx0, top + 1, wcut, False, work[(work > 0) & ~lds], c))
    return out


def house_plan(g, c, lds_min=None, max_ranges=None):
    """the plan of ensure_house_plan on g as numbered (lds_min None: no GM_RECT_LDS_MIN given -- the threshold per walk applies)"""
    rp, col, src = _csr(g)
    nv, deg = rp.size - 1, np.diff(rp)
    ids, T = c["house_ids"], c["one_task_rows"]
    n = (nv + ids - 1) // ids
    if max_ranges is not None:
        n = min(n, max_ranges)
    cut = max(0, nv - n * ids)
    keys_below_cut = np.bincount(src[col < cut], minlength=nv)
    work = np.bincount(src, weights=(deg[col] + 1), minlength=nv).astype(np.int64)
    wcut = np.bincount(src, weights=keys_below_cut[col], minlength=nv).astype(np.int64)
    per = np.where(deg <= c["house_fw16_rows"], 4, 2)
    need = np.full(nv, c["lds_min_default"] if lds_min is None else lds_min, dtype=np.int64)
    if lds_min is None:
        need = np.where(deg > T, need, np.maximum(need, c["house_walk_min_default"] * ((n + per - 1) // per)))
    lds = (work > 0) & (work >= need) & (n > 0)
    out = {"n": n, "cut": cut, "lds": lds, "deg": deg}
    out.update(_task_counts(lds, deg, np.full(nv, n), wcut + deg, True, work[(work > 0) & ~lds], c))
    return out


PLAN_KEYS = ("n", "cut", "rb", "lb", "lds_range_tasks", "lds_whole_tasks", "front_tasks", "front_heavy_tasks", "heavy_tasks", "light_tasks")


def plan_public(plan):
    """the part of a restated plan that gm_map_plan_info reports"""
    return {k: plan[k] for k in PLAN_KEYS if k in plan}


def rect_counters(g, plan):
    """per range k of the plan: {"max": the largest counter an LDS centre's walk leaves in it, "pair": whether two ends that SHARE A WORD of
    the map both reach it}.  A counter is c(v0, w) = the neighbours x < v0 of v0 that have the end w < v0."""
    rp, col, _ = _csr(g)
    rb, lb = np.asarray(plan["rb"]), plan["lb"]
    out = [{"max": 0, "pair": False} for _ in lb]
    for v0 in np.flatnonzero(plan["lds"]):
        rows = col[rp[v0]:rp[v0] + plan["idx0"][v0]]
        lens = rp[rows + 1] - rp[rows]
        first = np.zeros(rows.size, dtype=np.int64)
        np.cumsum(lens[:-1], out=first[1:])
        w = col[np.arange(int(lens.sum()), dtype=np.int64) + np.repeat(rp[rows] - first, lens)]
        w = w[(w < v0) & (w >= rb[0])]
        if w.size == 0:
            continue
        ends, cnt = np.unique(w, return_counts=True)
        ek = np.searchsorted(rb[1:], ends, side="right")
        for kk in np.unique(ek):
            m = ek == kk
            cmax = int(cnt[m].max())
            o = out[kk]
            if cmax > o["max"]:
                o["max"], o["pair"] = cmax, False
            if cmax == o["max"]:
                top = ends[m][cnt[m] == cmax] - rb[kk]
                per_word = 1 << (5 - lb[kk])
                o["pair"] |= per_word > 1 and bool((np.diff(top) == 1)[(top[:-1] % per_word) != per_word - 1].any())
    return out


# ---- the cells ------------------------------------------------------------------------------------------------------------------------------
@dataclass
class Cell:
    pattern: str                      # "rectangle" / "house"
    graph: object
    options: dict = field(default_factory=dict)   # developer options the cell's path needs (GM_RECT_LDS_MIN, GM_RECT_LDS_RANGES)
    claims: dict = field(default_factory=dict)    # sentence -> bool
    closed_form: int | None = None    # the count where a formula gives it
    slow_forms: bool = True           # run the nested / flat A/B forms too
    plans: dict = field(default_factory=dict)     # rectangle: {"default": .., "as numbered": ..}; house: {"default": ..}


def _opts(options):
    lds_min = int(options["GM_RECT_LDS_MIN"]) if "GM_RECT_LDS_MIN" in options else None
    mr = int(options["GM_RECT_LDS_RANGES"]) if "GM_RECT_LDS_RANGES" in options else None
    return lds_min, mr


def _rect_cell(g, c, options, closed_form=None, slow_forms=True):
    lds_min, mr = _opts(options)
    dc, _ = degree_copy(g)
    kw = dict(lds_min=lds_min, max_ranges=mr)
    return Cell("rectangle", g, dict(options), {}, closed_form, slow_forms, {"default": rect_plan(dc, c, **kw), "as numbered": rect_plan(g, c, **kw)})


def _house_cell(g, c, options, closed_form=None, slow_forms=True):
    lds_min, mr = _opts(options)
    return Cell("house", g, dict(options), {}, closed_form, slow_forms, {"default": house_plan(g, c, lds_min=lds_min, max_ranges=mr)})


def k3n(n, c, far_hub=0, lds_min_one=False, hubs=3):
    """K_{hubs, n}, the hubs on the last ids -- numbered ascending in degree, so the degree copy is the graph itself -- with isolated ids in
    front so that the first two hubs share a word of the map whatever its width: on the centre h2 (h1) the ends h0 and h1 (h0) count n.
    C(hubs, 2) C(n, 2) rectangles.  Where the graph is larger than the hubs' range, that range ends at the last id and the hubs' places in
    a word are fixed from the top: only with FOUR hubs do the first two share a word there (the 2^16 cells).  far_hub > 0: a star of that
    many leaves whose hub sits on the LAST id, more than four blocks of isolated ids above K_{3, n}: as numbered the star's range is wide
    and K_{3, n} lies in a range of its own width below; the degree copy moves everything together (correct, but the hubs share the star's
    range)."""
    pad = (-n) % 4
    first_hub = pad + n
    s = np.repeat(np.arange(pad, pad + n, dtype=np.int64), hubs)
    d = np.tile(first_hub + np.arange(hubs, dtype=np.int64), n)
    nv = first_hub + hubs
    if far_hub:
        gap = 4 * c["rect_block"] + 4 + (-far_hub) % 4   # (the ranges are whole blocks from the LAST id down: the hubs keep their place in a word)
        leaves = nv + gap + np.arange(far_hub, dtype=np.int64)
        nv = int(leaves[-1]) + 2
        s, d = np.concatenate([s, leaves]), np.concatenate([d, np.full(far_hub, nv - 1, dtype=np.int64)])
    g = _graph(nv, s, d)
    cell = _rect_cell(g, c, {"GM_RECT_LDS_MIN": "1"} if lds_min_one else {}, closed_form=comb(hubs, 2) * comb(n, 2))
    cell.hubs = first_hub + np.arange(hubs)
    return cell


def _width_claims(cell, c, n, copy):
    """the claims of a K_{3, n} width cell on one copy: which width the range of the hubs has, and that two ends sharing a word reach n"""
    g = cell.graph if copy == "as numbered" else degree_copy(cell.graph)[0]
    plan = cell.plans[copy]
    counters = rect_counters(g, plan)
    newid = np.arange(g.V()) if copy == "as numbered" else degree_copy(cell.graph)[1]
    hub = int(newid[cell.hubs[0]])
    k = int(np.searchsorted(np.asarray(plan["rb"][1:]), hub, side="right"))
    bits = 1 << plan["lb"][k]
    want_bits = 8 if n < 2 ** 8 else 16 if n < 2 ** 16 else 32
    T = c["one_task_rows"]
    out = {f"{copy}: the hubs' range has {want_bits}-bit counters": bits == want_bits,
           f"{copy}: the largest counter of that range is n = {n}": counters[k]["max"] == n,
           f"{copy}: the hubs are LDS centres": bool(plan["lds"][newid[cell.hubs[1:]]].all()),
           f"{copy}: the hubs are {'one task (RTN)' if n <= T else 'a task per range (read back)'}":
               (plan["lds_whole_tasks"] >= 2 and plan["lds_range_tasks"] == 0) if n <= T else plan["lds_range_tasks"] >= 2}
    if bits < 32:
        out[f"{copy}: two ends that share a word both reach it"] = counters[k]["pair"]
    if n in (2 ** 8 - 1, 2 ** 16 - 1):
        out[f"{copy}: that counter is the last value of its width"] = n == (1 << bits) - 1
    return out


def rect_width_cell(n, c, far=False, hubs=3):
    T = c["one_task_rows"]
    cell = k3n(n, c, far_hub=(HUB_ROWS if far else 0), lds_min_one=n * (hubs + 1) < c["lds_min_default"], hubs=hubs)
    copies = ("as numbered",) if far else ("default", "as numbered")
    for copy in copies:
        cell.claims.update(_width_claims(cell, c, n, copy))
    if far:
        plan = cell.plans["as numbered"]
        cell.claims["as numbered: a range of 8-bit counters below a wider one"] = plan["lb"][-1] == 4 and 3 in plan["lb"][:-1] if n < 2 ** 8 else plan["lb"][-1] == 4
    cell.slow_forms = n <= 4 * T  # (the flattened form intersects two lists for each of the 2^31 wedges of a hub: left out of the 2^16 cells)
    return cell


def rect_rows_cell(c):
    """ONE centre (the last id, one task) whose rows hold long_row - 1, long_row, long_row + 1 keys and the same around 4 long_row inside its
    range, and whose sixteen waves flatten totals from mark_window - 1 on (mark_window = one tile group today): row r of the centre goes to
    wave r mod 16, so the rows 16 j + w, j = 1 .. 8, hold long_row - 1 keys each and row w holds mark_window - 1 + w - 8 (long_row - 1) keys.
    Rows are the neighbours in id order, and the degree copy orders by degree = keys + 1: lengths ascend with the row.  The rows draw their keys
    from the front of one pool, so nearly every end is shared and the counters differ from end to end."""
    L, MW, waves = c["long_row"], c["mark_window"], c["one_task_rows"] // LANES
    per_wave = (MW - 1) // (L - 1)                      # rows of L - 1 keys below one window
    first = MW - 1 - per_wave * (L - 1)                 # keys of wave 0's first row
    assert first >= 1 and first + waves - 1 < L - 1, "the first rows stay the shortest"
    lens = [first + w for w in range(waves)] + [L - 1] * (per_wave * waves) + [L, L + 1, 4 * L - 1, 4 * L, 4 * L + 1]
    pool = 4 * L + 1
    nleaf = ((pool + 2 + waves - 1) // waves) * waves   # private leaves of the centre: it keeps the highest degree, and the rows their waves
    nrows = len(lens)
    leaf0, row0 = pool, pool + nleaf
    v0 = row0 + nrows
    s = [np.full(nleaf, v0, dtype=np.int64), np.full(nrows, v0, dtype=np.int64)]
    d = [leaf0 + np.arange(nleaf, dtype=np.int64), row0 + np.arange(nrows, dtype=np.int64)]
    for r, n in enumerate(lens):
        s.append(np.full(n, row0 + r, dtype=np.int64))
        d.append(np.arange(n, dtype=np.int64))
    g = _graph(v0 + 1, np.concatenate(s), np.concatenate(d))
    cell = _rect_cell(g, c, {"GM_RECT_LDS_MIN": "1"})
    for copy in ("default", "as numbered"):
        h, newid = (g, np.arange(g.V())) if copy == "as numbered" else degree_copy(g)
        plan = cell.plans[copy]
        rp, col, _ = _csr(h)
        centre = int(newid[v0])
        rows = col[rp[centre]:rp[centre] + plan["idx0"][centre]]
        keys = np.array([int((col[rp[x]:rp[x + 1]] < centre).sum()) for x in rows])
        wave_total = np.array([int(keys[w::waves][keys[w::waves] < L].sum()) for w in range(waves)])
        cell.claims.update({
            f"{copy}: the centre is the last id, one task, one range": centre == h.V() - 1 and plan["n"] == 1 and bool(plan["lds"][centre]) and plan["idx0"][centre] <= c["one_task_rows"],
            f"{copy}: rows of long_row - 1, long_row, long_row + 1 keys": {L - 1, L, L + 1} <= set(keys.tolist()),
            f"{copy}: rows of 4 long_row - 1, 4 long_row, 4 long_row + 1 keys": {4 * L - 1, 4 * L, 4 * L + 1} <= set(keys.tolist()),
            f"{copy}: waves flatten mark_window - 1, mark_window, mark_window + 1 keys": {MW - 1, MW, MW + 1} <= set(wave_total.tolist()),
            f"{copy}: ... and a whole tile group and one key more": {c["tile_group"], c["tile_group"] + 1} <= set(wave_total.tolist()),
        })
    return cell


def _c4_centre(h, v):
    """v has exactly two neighbours below it and they share an end below v: v is the centre of a 4-cycle the walk counts at v"""
    rp, col, _ = _csr(h)
    nb = col[rp[v]:rp[v + 1]]
    rows = nb[nb < v]
    if rows.size != 2:
        return False
    common = np.intersect1d(col[rp[rows[0]]:rp[rows[0] + 1]], col[rp[rows[1]]:rp[rows[1] + 1]])
    return bool((common < v).any())


def rect_cut_cell(max_ranges, c):
    """More ids than GM_RECT_LDS_RANGES = max_ranges ranges cover, so that the walk of an LDS centre is SPLIT: its ends from the cut on count in
    rect_lds_kernel, those below stay with rect_acc_kernel (the front of its list).  From the first id up, in the order of the degree copy:
      leaves    of the rows under G0 / G1 (degree 1)
      the zone  of vertices of degree 2: hub ends (joined to the two rows of one pair of X: 2 2-paths and 1 rectangle with every hub), the
                4-cycles C4 = (end, row, row, centre) on four ids of their own, and the vertices between strung on one long cycle
      rows      under G0 / G1, the rows X under the hubs, three hubs (every hub joined to every row of X; the middle one misses the last)
      G1, G0    on the last ids: joined to heavy_centre / ROW_WEIGHT rows of d(x) + 1 = ROW_WEIGHT, but for one row each: G0's estimate of
                2-paths is exactly heavy_centre -- a workgroup of its own where every end goes to the global maps -- and G1's heavy_centre - 1
    The cut lies inside the zone.  heavy_centre / 2 hub ends lie below it: two hubs keep exactly heavy_centre 2-paths for the FRONT of
    rect_acc_kernel and the middle hub heavy_centre - 1.  Centres that carry a 4-cycle, LDS centres under GM_RECT_LDS_MIN = 1 where they
    lie above the cut: a C4 on the first ids of the zone (below the cut) in both cells; one range: a C4 whose centre is the id `cut` itself
    (not above the cut: it stays on the rest list) and one whose centre is cut + 1 with every end below the cut (its walk of range 0 finds
    only itself, dropped by value); two ranges: a C4 with the centre on cut + 1, its rows below the cut and its one end ON the cut, and hub
    ends on the last id of range 0 and the first of range 1.  (Centre-on-cut and end-on-cut need the same id: one cell each.)"""
    W, heavy = c["rect_block"], c["heavy_centre"]
    nx, nh, per = HUB_ROWS, 3, ROW_WEIGHT
    m = heavy // per                                           # rows of G0 and of G1
    assert m * per == heavy and m > per and per > 3
    nl = (m - 1) * (per - 3) + (per - 2) + (per - 3)           # shared rows: G0, G1 + per - 3 leaves; G0's own: per - 2; G1's own: per - 3
    top = (m + 1) + nx + nh + 2                                # everything above the zone
    covered = 2 * W + (4 * W if max_ranges > 1 else 0)         # degrees from 2^8 on in the top block: 16 bits there, 8 bits below
    below = heavy // 2                                         # hub ends below the cut: 2 2-paths each with every hub
    z0 = nl
    cut = z0 + CUT_MARGIN + below
    nv = cut + covered
    z1 = nv - top                                              # the zone is [z0, z1)
    assert z0 + 4 < cut - 10 - below and cut + 16 < z1
    c4 = [(z0, z0 + 1, z0 + 2, z0 + 3)]                        # (end, row, row, centre)
    if max_ranges == 1:
        c4 += [(cut - 8, cut - 7, cut - 6, cut), (cut - 5, cut - 4, cut - 3, cut + 1)]
        above = [cut + 2, cut + 9, z1 - 2, z1 - 1]
    else:
        c4 += [(cut, cut - 7, cut - 6, cut + 1)]
        rb1 = nv - 2 * W
        above = [cut + 2, cut + 9, rb1 - 1, rb1, z1 - 2, z1 - 1]
    ends = np.concatenate([np.arange(cut - 10 - (below - 2), cut - 10), [cut - 2, cut - 1], above]).astype(np.int64)
    RG = z1 + np.arange(m + 1, dtype=np.int64)                 # G1's own row first (the lowest degree), the shared rows, G0's own row
    X = RG[-1] + 1 + np.arange(nx, dtype=np.int64)
    H = X[-1] + 1 + np.arange(nh, dtype=np.int64)
    G1, G0 = nv - 2, nv - 1
    npair = nx // 2 - 1                                        # the pairs (0, 1) .. ; the last pair is kept for ONE end below the cut
    pair = np.arange(ends.size) % npair
    pair[0] = npair                                            # (the end on the lowest id goes to the last pair: rows nx - 2, nx - 1)
    s = [np.repeat(ends, 2)]
    d = [np.stack([X[2 * pair], X[2 * pair + 1]], axis=1).ravel()]
    for i, h in enumerate(H):
        rows = X[:-1] if i == 1 else X
        s.append(np.full(rows.size, h, dtype=np.int64))
        d.append(rows)
    for w, ra, rb_, v in c4:
        s.append(np.array([w, w, v, v], dtype=np.int64))
        d.append(np.array([ra, rb_, ra, rb_], dtype=np.int64))
    used = np.concatenate([ends, np.array(c4, dtype=np.int64).ravel()])
    assert np.unique(used).size == used.size
    pads = np.setdiff1d(np.arange(z0, z1, dtype=np.int64), used)
    s.append(pads)
    d.append(np.roll(pads, -1))
    s += [np.full(m, G1, dtype=np.int64), np.full(m, G0, dtype=np.int64)]
    d += [RG[:-1], RG[1:]]
    nleaf = np.concatenate([[per - 3], np.full(m - 1, per - 3), [per - 2]])
    s.append(np.repeat(RG, nleaf))
    d.append(np.arange(nl, dtype=np.int64))
    g = _graph(nv, np.concatenate(s), np.concatenate(d))
    # (the flattened form runs too: a hub has C(HUB_ROWS, 2), G0 C(heavy_centre / ROW_WEIGHT, 2) wedges)
    cell = _rect_cell(g, c, {"GM_RECT_LDS_RANGES": str(max_ranges), "GM_RECT_LDS_MIN": "1"})
    centres = {f"{x[3] - cut:+d}" if abs(x[3] - cut) < 4 else "first ids of the zone": x[3] for x in c4}
    for copy in ("default", "as numbered"):
        h, newid = (g, np.arange(nv)) if copy == "as numbered" else degree_copy(g)
        plan = cell.plans[copy]
        zone = np.arange(z0, z1)
        cell.claims.update({
            f"{copy}: {max_ranges} range(s), the cut inside the zone": plan["n"] == max_ranges and plan["cut"] == cut and plan["lb"][-1] == 4 and z0 < cut < z1,
            f"{copy}: the zone keeps its ids": bool((newid[zone] == zone).all()),
            f"{copy}: hub ends on cut - 1 (the last below) and cut + 2": {cut - 1, cut + 2} <= set(ends.tolist()),
            f"{copy}: the hubs are one-task LDS centres": bool(plan["lds"][newid[H]].all()) and bool((plan["idx0"][newid[H]] <= c["one_task_rows"]).all()),
            f"{copy}: two hubs keep heavy_centre 2-paths below the cut, one heavy_centre - 1":
                sorted(plan["wcut"][newid[H]].tolist()) == [heavy - 1, heavy, heavy] and plan["front_heavy_tasks"] == 2,
            f"{copy}: G0's 2-paths are heavy_centre, G1's heavy_centre - 1 (both have more rows than one task takes)":
                [int(plan["work"][newid[G1]]), int(plan["work"][newid[G0]])] == [heavy - 1, heavy] and bool((plan["idx0"][newid[[G1, G0]]] > c["one_task_rows"]).all()),
            f"{copy}: a C4 centre below the cut stays on the rest list": _c4_centre(h, c4[0][3]) and c4[0][3] < cut and not plan["lds"][c4[0][3]] and plan["work"][c4[0][3]] > 0,
        })
        if max_ranges == 1:
            cell.claims.update({
                f"{copy}: a C4 centre ON the cut stays on the rest list": _c4_centre(h, cut) and not plan["lds"][cut] and plan["work"][cut] > 0,
                f"{copy}: a C4 centre on cut + 1 is an LDS centre with every end below the cut": _c4_centre(h, cut + 1) and bool(plan["lds"][cut + 1]) and plan["wcut"][cut + 1] == 2,
            })
        else:
            cell.claims.update({
                f"{copy}: a C4 centre on cut + 1 is an LDS centre with its one end ON the cut": _c4_centre(h, cut + 1) and bool(plan["lds"][cut + 1]) and plan["wcut"][cut + 1] == 0
                and cut in h.col_idx[h.row_ptr[cut - 7]:h.row_ptr[cut - 6]].tolist(),
                f"{copy}: hub ends on the last id of range 0 and the first of range 1": plan["rb"][1] == rb1 and {rb1 - 1, rb1} <= set(ends.tolist()),
            })
    cell.centres = centres
    return cell


def rect_range_edges_cell(c):
    """AS NUMBERED (the degree copy packs every vertex with an edge into the top range): three ranges of 16-bit counters, ends on the first
    and the last id of each and on both sides of every boundary, and two centres INSIDE a range with ends on v0 - 1 and v0 + 1: a one-task
    centre (keys >= v0 dropped by value) and one with more rows than one task takes (the range's rows clipped by bisection).  Rows: ids from 8 on;
    every row is joined to every end and to the centres it belongs to."""
    W, T = c["rect_block"], c["one_task_rows"]
    nv = 6 * W - 100
    rb = [0, nv - 4 * W, nv - 2 * W, nv]
    c1, c2 = rb[1] + 500, rb[2] + 700                         # one task / a task per range
    nx = T + 6
    X = 8 + np.arange(nx, dtype=np.int64)
    ends = sorted({0, rb[1] - 1, rb[1], rb[2] - 1, rb[2], c1 - 1, c1 + 1, c2 - 1, c2 + 1, nv - 2})
    ends = np.array(ends, dtype=np.int64)
    top = nv - 1                                              # a centre above every end: the last id of the top range is its own
    s = [np.repeat(X, ends.size), X[:T // 2], X, X]
    d = [np.tile(ends, nx), np.full(T // 2, c1, dtype=np.int64), np.full(nx, c2, dtype=np.int64), np.full(nx, top, dtype=np.int64)]
    g = _graph(nv, np.concatenate(s), np.concatenate(d))
    cell = _rect_cell(g, c, {})
    plan = cell.plans["as numbered"]
    counters = rect_counters(g, plan)
    cell.claims = {
        "as numbered: three ranges of 16-bit counters": plan["rb"] == rb and plan["lb"] == [4, 4, 4],
        "as numbered: ends on the first and the last id of every range (the last id of the graph is a centre)":
            all(rb[k] in ends and (rb[k + 1] - 1 in ends or k == 2) for k in range(3)) and nv - 2 in ends,
        "as numbered: a one-task centre inside range 1 with ends on v0 - 1 and v0 + 1": plan["idx0"][c1] <= T and bool(plan["lds"][c1]) and rb[1] < c1 < rb[2],
        "as numbered: a centre with a task per range inside range 2 with ends on v0 - 1 and v0 + 1": plan["idx0"][c2] > T and bool(plan["lds"][c2]) and rb[2] < c2 < nv,
        "as numbered: both kinds of task": plan["lds_range_tasks"] >= 6 and plan["lds_whole_tasks"] >= 1,
        "as numbered: every range holds a counter of all the rows": all(k["max"] == nx for k in counters),
    }
    return cell


# ---- house -----------------------------------------------------------------------------------------------------------------------------------
def house_saturation_cell(m, c):
    """K_m, every vertex of it joined to three twins that are not adjacent to each other, the twins on the LAST ids, the first two of them on
    ids that share a map word: on each twin centre v0 the other twins are ends with n = m 2-paths whose weights t(v0, x) = m - 1 sum to
    S = m (m - 1) -- the last values 6 + 10 bits hold at m = house_fw16_rows, and 11 + 21 bits at m = one_task_rows.  The clique's vertices have
    m + 2 neighbours: above one_task_rows - 2 they are centres with a task per range, in the same call."""
    pad = m % 2
    tw = m + pad + np.arange(3, dtype=np.int64)
    i, j = np.triu_indices(m, 1)
    s = np.concatenate([i.astype(np.int64), np.repeat(np.arange(m, dtype=np.int64), 3)])
    d = np.concatenate([j.astype(np.int64), np.tile(tw, m)])
    g = _graph(int(tw[-1]) + 1, s, d)
    F16, T = c["house_fw16_rows"], c["one_task_rows"]
    cell = _house_cell(g, c, {"GM_RECT_LDS_MIN": "1"} if m * (m + 3) < 4 * c["lds_min_default"] else {}, slow_forms=m <= 4 * F16)
    plan = cell.plans["default"]
    bits = (6, 10) if m <= F16 else (11, 21) if m <= T else (24, 40)
    cell.claims = {
        "the twins are LDS centres with m rows": bool(plan["lds"][tw].all()) and bool((plan["deg"][tw] == m).all()),
        f"a twin is {'one task' if m <= T else 'a task per range'}": (plan["lds_whole_tasks"] >= 3) if m <= T else plan["lds_range_tasks"] >= 3 * plan["n"],
        f"n = m and S = m (m - 1) fit {bits[0]} + {bits[1]} bits": m < 2 ** bits[0] and m * (m - 1) < 2 ** bits[1],
        "the first two twins share a 32-bit word of 16-bit fields (and a 64-bit word of 32-bit fields)": int(tw[0]) % 2 == 0,
        "one range": plan["n"] == 1 and plan["cut"] == 0,
    }
    if m == F16:
        cell.claims["n and S are exactly tight: one more row needs the next width"] = (m + 1) * m >= 2 ** bits[1]
    if m + 2 > T:
        cell.claims["the clique's vertices are centres with a task per range"] = plan["lds_range_tasks"] >= m
    cell.twins = tw
    return cell


def house_ranges_cell(n_ranges, m, c):
    """n_ranges ranges of house_ids ids (the last one a single id short), K_m on the ids 1 .. m, and twins joined to all of K_m on the first and
    the last id of EVERY range -- so on both sides of every boundary a walk joins or stops at -- and a centre twin on the last id but one of the
    graph.  m <= house_fw16_rows: four ranges per walk; above: two."""
    ids = c["house_ids"]
    nv = n_ranges * ids - 1
    edges = sorted({0, nv - 1, nv - 2} | {k * ids for k in range(1, n_ranges)} | {k * ids - 1 for k in range(1, n_ranges)})
    tw = np.array([e for e in edges if not 1 <= e <= m], dtype=np.int64)
    i, j = np.triu_indices(m, 1)
    s = np.concatenate([1 + i.astype(np.int64), np.repeat(1 + np.arange(m, dtype=np.int64), tw.size)])
    d = np.concatenate([1 + j.astype(np.int64), np.tile(tw, m)])
    g = _graph(nv, s, d)
    cell = _house_cell(g, c, {"GM_RECT_LDS_MIN": "1"})
    plan = cell.plans["default"]
    per = 4 if m <= c["house_fw16_rows"] else 2
    rb = [min(k * ids, nv) for k in range(n_ranges + 1)]
    cell.claims = {
        f"{n_ranges} ranges from id 0": plan["n"] == n_ranges and plan["cut"] == 0,
        f"the twins are one-task centres of {m} rows: {per} ranges per walk": bool(plan["lds"][tw].all()) and bool((plan["deg"][tw] == m).all()) and m <= c["one_task_rows"]
        and (m <= c["house_fw16_rows"]) == (per == 4),
        "twin ends on the first and the last id of every range": all(rb[k] in tw.tolist() and rb[k + 1] - 1 in tw.tolist() for k in range(n_ranges)),
        "the last centre has its own id among the keys and ends in every range": int(tw[-1]) == nv - 1 and tw.size >= 2 * n_ranges,
    }
    cell.twins = tw
    return cell


def house_long_rows_cell(q, keys, c):
    """A one-task centre v0 (the last id) beside q rows of exactly `keys` keys inside its one range: X = q row vertices on the first ids, each
    joined to v0 and to the first keys - 1 vertices of Y; v0 is joined to every second vertex of Y too, so that t(v0, x) > 0 weighs every
    2-path.  The vertices of Y are one-task centres with the same q rows.  keys = house_wg_row - 1 / house_wg_row: the wave strides the row
    itself / the row goes to the workgroup's queue; q = house_wg_queue - 1, house_wg_queue, beyond: the queue fills and the surplus falls back
    to the owning wave."""
    ny = keys - 1
    X = np.arange(q, dtype=np.int64)
    Y = q + np.arange(ny, dtype=np.int64)
    v0 = q + ny
    s = np.concatenate([np.repeat(X, ny), X, Y[::2]])
    d = np.concatenate([np.tile(Y, q), np.full(q, v0, dtype=np.int64), np.full(Y[::2].size, v0, dtype=np.int64)])
    g = _graph(v0 + 1, s, d)
    cell = _house_cell(g, c, {} if q > 8 else {"GM_RECT_LDS_MIN": "1"}, slow_forms=q <= 8)
    plan = cell.plans["default"]
    rp, col, _ = _csr(g)
    rows = col[rp[v0]:rp[v0 + 1]]
    lens = (rp[rows + 1] - rp[rows])
    Q, WG = c["house_wg_queue"], c["house_wg_row"]
    nq = int((lens >= WG).sum())
    cell.claims = {
        "v0 is a one-task LDS centre, one range": bool(plan["lds"][v0]) and plan["deg"][v0] <= c["one_task_rows"] and plan["n"] == 1,
        f"v0 has {q} rows of {keys} keys": int((lens == keys).sum()) == q and nq == (q if keys >= WG else 0),
        "the rows of v0 are below it and carry weight": bool((rows[:q] < v0).all()) and ny >= 2,
        f"rows that reach the queue: {q if keys >= WG else 0}, of them past its slots: {max(q - Q, 0) if keys >= WG else 0}": nq == (q if keys >= WG else 0),
    }
    cell.v0 = v0
    return cell


def house_cut_cell(c):
    """GM_RECT_LDS_RANGES = 1 on more than house_ids ids: the one range covers the last house_ids ids and the ends below its first id, the cut,
    stay with house_acc_kernel.  Y on the first ids, isolated ids, q rows X, the centre v0 last; the cut falls in the middle of Y, so ends with
    weight lie on cut - 1 and on cut.  v0 and the vertices of Y keep q |Y| / 2 2-paths below the cut, past heavy_centre: a workgroup each in
    the front of house_acc_kernel; the rows X keep none: light front tasks."""
    ids, heavy = c["house_ids"], c["heavy_centre"]
    ny = c["house_wg_row"] - 2                                 # Y: rows X of ny + 1 keys stay below the work-group queue
    q = 2 * ((heavy + ny - 1) // ny) + 2                       # rows: q ny / 2 2-paths below the cut pass heavy_centre
    cut = ny // 2
    nv = cut + ids
    Y = np.arange(ny, dtype=np.int64)
    X = nv - 1 - q + np.arange(q, dtype=np.int64)
    v0 = nv - 1
    s = np.concatenate([np.repeat(X, ny), X, Y[::2]])
    d = np.concatenate([np.tile(Y, q), np.full(q, v0, dtype=np.int64), np.full(Y[::2].size, v0, dtype=np.int64)])
    g = _graph(nv, s, d)
    cell = _house_cell(g, c, {"GM_RECT_LDS_RANGES": "1"}, slow_forms=False)
    plan = cell.plans["default"]
    cell.claims = {
        "one range, the cut in the middle of Y": plan["n"] == 1 and plan["cut"] == cut and 0 < cut < ny,
        "ends with weight on cut - 1 and on cut (Y fills the ids below and from the cut on)": cut - 1 in Y and cut in Y and ny >= 2,
        "v0 is a one-task LDS centre past heavy_centre in the front": q * cut + plan["deg"][v0] >= heavy and plan["deg"][v0] <= c["one_task_rows"],
        "whole-workgroup and four-to-a-task centres in the front": plan["front_heavy_tasks"] >= 1 and plan["front_tasks"] > plan["front_heavy_tasks"],
        "the vertices of Y below the cut are LDS centres too (every centre's ends above the cut are in the range)": bool(plan["lds"][Y].all()),
    }
    cell.v0 = v0
    return cell


# ---- the table -----------------------------------------------------------------------------------------------------------------------------
# (the names say which side of which size; the sizes themselves come from the library when a cell is built)
RECT_CELLS = ["rect-width-2^8-1", "rect-width-2^8", "rect-width-2^8-1-far-hub", "rect-width-2^8-far-hub", "rect-one-task-rows", "rect-one-task-rows+1",
              "rect-width-2^16-1", "rect-width-2^16", "rect-rows", "rect-range-edges", "rect-cut-1-range", "rect-cut-2-ranges"]
HOUSE_CELLS = (["house-fields-fw16", "house-fields-fw16+1", "house-fields-one-task", "house-fields-one-task+1"]
               + [f"house-ranges-{n}-{kind}" for n in (1, 2, 3, 4, 5) for kind in ("fw16", "fw32")]
               + ["house-row-wg-1", "house-row-wg", "house-queue-1", "house-queue", "house-queue+8", "house-cut"])
CELLS = RECT_CELLS + HOUSE_CELLS
MANY_VERTICES = 5000     # vertices of degree >= 2 from which the total comes from rect_local_ref.total_by_pairs (one bincount per vertex otherwise)
BIG_REFERENCE = 100_000   # entries from which a cell with a closed form is held against that alone (rect_local_ref walks every 2-path)


def build(name, c):
    T, F16, Q, WG = c["one_task_rows"], c["house_fw16_rows"], c["house_wg_queue"], c["house_wg_row"]
    side = 1 if name.endswith("+1") else 0
    if name.startswith("rect-width-2^8"):
        return rect_width_cell(2 ** 8 - 1 + ("2^8-1" not in name), c, far="far-hub" in name)
    if name.startswith("rect-width-2^16"):   # (four hubs: see k3n)
        return rect_width_cell(2 ** 16 - 1 + ("2^16-1" not in name), c, hubs=4)
    if name.startswith("rect-one-task-rows"):
        return rect_width_cell(T + side, c)
    if name == "rect-rows":
        return rect_rows_cell(c)
    if name == "rect-range-edges":
        return rect_range_edges_cell(c)
    if name.startswith("rect-cut-"):
        return rect_cut_cell(int(name.split("-")[2]), c)
    if name == "house-cut":
        return house_cut_cell(c)
    if name.startswith("house-fields-fw16"):
        return house_saturation_cell(F16 + side, c)
    if name.startswith("house-fields-one-task"):
        return house_saturation_cell(T + side, c)
    if name.startswith("house-ranges-"):
        _, _, n, kind = name.split("-")
        return house_ranges_cell(int(n), F16 // 4 if kind == "fw16" else F16 + 8, c)
    if name.startswith("house-row-wg"):
        return house_long_rows_cell(2, WG - (1 if name.endswith("-1") else 0), c)
    if name.startswith("house-queue"):
        return house_long_rows_cell(Q + (8 if name.endswith("+8") else -1 if name.endswith("-1") else 0), WG, c)
    raise KeyError(name)


def reference(cell):
    """the count the cell must give: tests/rect_local_ref.py / tests/house_ref.py on the whole graph; a large cell with a closed form is held
    against the formula (the host test holds the formula against the reference on the small cells of the same family)"""
    import house_ref as H
    import rect_local_ref as R

    if cell.pattern == "house":
        return H.house(cell.graph)
    if cell.closed_form is not None and cell.graph.E() >= BIG_REFERENCE:
        return cell.closed_form
    if int((np.diff(cell.graph.row_ptr) >= 2).sum()) > MANY_VERTICES:
        return R.total_by_pairs(cell.graph)
    return R.total(R.rect_local(cell.graph)[1])


def constants():
    """the sizes the library exports (needs the built library, not a GPU)"""
    from graphminer_amd import map_constants

    return map_constants()
