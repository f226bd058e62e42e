"""The batch lengths at which the flattened pass of tch_kernel (gm_tch.hip) changes form (test helper; imported by
tests/test_probe_flat_groups_host.py and tests/test_gpu_tch_flat_groups.py).

A batch of tests/probe_graphs.py `batch(M, ell)` is 64 lists of `ell` keys: 64 * ell flattened positions.  The pass walks them in tile
groups of G = 256 positions beside the 1024-bucket table (M = 1024) and 512 beside the 2048-bucket one (M = 2048), inside mark windows of
W = 8192 and 4096 positions.  Every group that lies wholly below the total runs in the peeled form (no range test), the last group of a
window, if it is partial, in the guarded form; `where(M, ell)` names the place the total lands at."""
GROUP = {1024: 256, 2048: 512}     # kTchFlatTilesSmall / kTchFlatTilesBig tiles of 64
WINDOW = {1024: 8192, 2048: 4096}  # TchLds::kBitWindow
TILE = 64

# ell -> what 64 * ell is meant to be, per M (asserted by the host test)
CASES = {
    1024: {36: "group boundary", 35: "one tile short of a group", 37: "one tile past a group", 40: "group boundary",
           39: "one tile short of a group", 41: "one tile past a group", 63: "one tile short of a group", 65: "one tile past a group",
           124: "one group short of the window", 132: "one group past the window", 127: "one tile short of the window",
           129: "one tile past the window"},
    2048: {40: "group boundary", 39: "one tile short of a group", 41: "one tile past a group", 36: "half a group",
           35: "three tiles into a group", 37: "five tiles into a group", 63: "one tile short of the window", 65: "one tile past the window",
           124: "past the window, half a group", 132: "two windows and half a group"},
}
PARAMS = [(M, ell) for M in CASES for ell in sorted(CASES[M])]


def where(M: int, ell: int) -> str:
    """the place 64 * ell lands at, worked out from the kernel's constants"""
    total, G, W = 64 * ell, GROUP[M], WINDOW[M]
    tiles_in = (total % G) // TILE  # whole tiles of the last, partial group (the lengths used are whole tiles: 64 lists)
    assert total % TILE == 0
    if total == W - G:
        return "one group short of the window"
    if total == W + G:
        return "one group past the window"
    if total == W - TILE:
        return "one tile short of the window"
    if total == W + TILE:
        return "one tile past the window"
    if total > W:
        rest = total % W
        half = "half a group" if rest % G == G // 2 else f"{(rest % G) // TILE} tiles into a group"
        return ("past the window, " if total < 2 * W else "two windows and ") + half
    if tiles_in == 0:
        return "group boundary"
    if tiles_in == G // TILE - 1:
        return "one tile short of a group"
    if tiles_in == 1:
        return "one tile past a group"
    if tiles_in * 2 == G // TILE:
        return "half a group"
    return {3: "three tiles into a group", 5: "five tiles into a group"}[tiles_in]
